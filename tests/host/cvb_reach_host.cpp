// Host replay of the batch verifier's Fr kernels (csrc/circuit_verify_kernels.hip: k_cvb_public, k_cvb_lin, k_cvb_scalars, cvb_plain,
// cvb_is_zero, glv_split_device) on the unchanged csrc/fr30.hip.h, for tests/test_cvb_extremes.py: a stand-alone program (plain g++
// -O2 -fwrapv; the header is __host__ __device__ code).  Test infrastructure only; nothing is loaded into Python.
//
// It replays one proof per input record in the kernels' order of products, sums, negations and carry passes, not their memory
// layout: all 64 lanes of one workgroup of k_cvb_public in a loop (cvb_group_inverse's two scans, the substituted denominators, the
// hit, the 63 additions of the lanes' totals), one lane of k_cvb_lin (its shared inversion taken as fr30_inv of the lane's own
// denominator) and every lane q of k_cvb_scalars.  w, 1 + w, 1 / n and w^64 are INPUTS, so the test can make them extremal.
//
// stdin:   variant t lg_n e g n_public count
//          g t exponents
//          w w1 invn w64 shift_0 .. shift_(t-1)       (blst_fr images of the plain values, 64 hex digits each; prepared with
//                                                      fr30_arg_from_mont256 as the host prepares the kernels' constants)
//          count records: beta gamma alpha zeta v rho, the 2 t evaluations, the n_public public inputs (blst_fr images)
// variant: 0 the kernels; 1 and 2 are WEAKENED (never on a device): 1 makes the zero tests on the unreduced difference
//          (fr30_to_limbs(z - w) in the place of cvb_is_zero(d)), 2 hands fr30_to_limbs the raw sum g0 + g1 of G1's term of P1 without
//          the reducing product (its line then holds the canonical residue of the multiplier form, rho left out).
// stdout:  kR9SumRawBound and kR9SumNormBound as the header states them.  Then one line of numbers: per named sum (enum Sum) the
//          largest |digit 0..7| entering its carry pass, then per sum the largest |digit 8| leaving it; the largest |digit 0..7| of any
//          product, load or carry pass; the largest |digit 8| of any product; the largest |column| of any product (exact, saturated at
//          2^64 - 1); the smallest and the largest value handed to fr30_to_limbs in units of r / 2^20 (rounded towards zero); how many
//          of them were outside (-r, 2r), how many were -r itself and how many r itself, exactly; the largest |p| - |a| |b| / 2^270 of
//          any product p = a b / 2^270 in units of r / 2^20 (rounded up): the part of a product's bound that is its own.
//          Then per record: "pi <plain> <hit or -1>", "lin" and four plain values, and Q lines "s <plain> <k1> <k2>" (a split scalar) or
//          "r <plain>" (a term of the key's row), lane by lane.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../kzg_poly_commit_exploration_amd/csrc/fr30.hip.h"
#include "../../kzg_poly_commit_exploration_amd/csrc/host_fr.hpp"
#include "../../kzg_poly_commit_exploration_amd/csrc/fr30_host.hpp"

using namespace kzg;

namespace {

// z - w^i; PI's running sum; the 64 lanes' total; zeta^n - 1 and zeta - 1; abar + gamma; a factor of A or B; [z]'s scalar; the constant
// of r; the g0 chain; g0 + g1 and P0's sum of the two
enum Sum { kZw = 0, kAcc, kTotal, kZn1, kAg, kFactor, kScZ, kKonst, kG0, kG01, kSums };
enum { kRaw = 0, kTop = kSums, kNorm = 2 * kSums, kProdTop, kColumn, kReports };
uint64_t rep[kReports];
int variant = 0;
void see(int which, int64_t v) {
    const uint64_t m = v < 0 ? (uint64_t)(-v) : (uint64_t)v;
    if (m > rep[which]) rep[which] = m;
}
void digits(const Fr30& v, int top) {
    for (int i = 0; i < kR9 - 1; i++) see(kNorm, v.d[i]);
    if (top >= 0) see(top, v.d[kR9 - 1]);
}
void column(__int128 acc) {
    const __int128 m = acc < 0 ? -acc : acc;
    const uint64_t s = m > (__int128)UINT64_MAX ? UINT64_MAX : (uint64_t)m;
    if (s > rep[kColumn]) rep[kColumn] = s;
}
// a lazy value in units of r
long double in_r(const Fr30& v) {
    long double x = 0, rr = 0;
    for (int i = kR9 - 1; i >= 0; i--) {
        x = x * 1073741824.0L + v.d[i];
        rr = rr * 1073741824.0L + fr30_rd(i);
    }
    return x / rr;
}
long double own_r = 0;
// fr30_mul with its columns followed in exact arithmetic; the product itself is the header's
Fr30 mul(const Fr30& a, const Fr30& b) {
    int32_t m[kR9];
    __int128 acc = 0;
    for (int k = 0; k < kR9; k++) {
        for (int i = 0; i <= k; i++) acc += (__int128)a.d[i] * b.d[k - i];
        for (int j = 0; j < k; j++) acc += (__int128)m[j] * fr30_rd(k - j);
        column(acc);
        m[k] = fr30_sext30(0u - (uint32_t)(uint64_t)acc);
        acc += m[k];
        acc >>= kR9Bits;
    }
    for (int k = kR9; k < 2 * kR9 - 1; k++) {
        for (int i = k - kR9 + 1; i < kR9; i++) acc += (__int128)a.d[i] * b.d[k - i];
        for (int j = k - kR9 + 1; j < kR9; j++) acc += (__int128)m[j] * fr30_rd(k - j);
        column(acc);
        acc = (acc + (1 << (kR9Bits - 1))) >> kR9Bits;
    }
    const Fr30 p = fr30_mul(a, b);
    digits(p, kProdTop);
    {  // |a| |b| / 2^270 in units of r: |a / r| |b / r| r / 2^270
        long double r270 = 1;
        for (int i = kR9 - 1; i >= 0; i--) r270 = r270 * 1073741824.0L;  // 2^270
        long double rr = 0;
        for (int i = kR9 - 1; i >= 0; i--) rr = rr * 1073741824.0L + fr30_rd(i);
        const long double pa = in_r(a), pb = in_r(b), pp = in_r(p);
        const long double own = (pp < 0 ? -pp : pp) - (pa < 0 ? -pa : pa) * (pb < 0 ? -pb : pb) * (rr / r270);
        if (own > own_r) own_r = own;
    }
    return p;
}
// sum `which`: a + sign b digit-wise, carry-normalised (fr30_add, fr30_sub); the raw digits reported in 64 bits, wrapped to 32 as the
// device would
Fr30 add(Sum which, const Fr30& a, const Fr30& b, int sign = 1) {
    Fr30 r;
    for (int i = 0; i < kR9; i++) {
        const int64_t s = (int64_t)a.d[i] + sign * (int64_t)b.d[i];
        if (i < kR9 - 1) see(kRaw + which, s);
        r.d[i] = (int32_t)(uint32_t)(uint64_t)s;
    }
    r = fr30_norm(r);
    digits(r, kTop + which);
    return r;
}
Fr30 neg(const Fr30& a) {
    Fr30 r;
    for (int i = 0; i < kR9; i++) r.d[i] = -a.d[i];
    return r;
}

// what fr30_to_limbs is handed: the sign of v - k r, exactly (sequential carry to unsigned digits with a signed top digit)
int sign_minus_kr(const Fr30& v, int k) {
    int64_t c = 0;
    bool nonzero = false;
    for (int i = 0; i < kR9 - 1; i++) {
        const int64_t t = (int64_t)v.d[i] - (int64_t)k * (int64_t)fr30_ru(i) + c;
        nonzero = nonzero || (t & kR9Mask);
        c = t >> kR9Bits;
    }
    const int64_t top = (int64_t)v.d[kR9 - 1] - (int64_t)k * (int64_t)fr30_ru(kR9 - 1) + c;
    return top < 0 ? -1 : (top > 0 || nonzero ? 1 : 0);
}
long double lo_r = 0, hi_r = 0;
uint64_t outside = 0, at_minus_r = 0, at_plus_r = 0;
void to_limbs(const Fr30& v, uint32_t l[8]) {
    const long double x = in_r(v);
    if (x < lo_r) lo_r = x;
    if (x > hi_r) hi_r = x;
    if (sign_minus_kr(v, -1) <= 0 || sign_minus_kr(v, 2) >= 0) outside++;
    if (sign_minus_kr(v, -1) == 0) at_minus_r++;
    if (sign_minus_kr(v, 1) == 0) at_plus_r++;
    fr30_to_limbs(v, l);
}
void cvb_plain(const Fr30& a, uint32_t l[8]) { to_limbs(mul(a, fr30_small(1)), l); }
bool all_zero(const uint32_t l[8]) { return (l[0] | l[1] | l[2] | l[3] | l[4] | l[5] | l[6] | l[7]) == 0; }
bool cvb_is_zero(const Fr30& a) {
    uint32_t l[8];
    cvb_plain(a, l);
    return all_zero(l);
}
// the kernels' d = cvb_mul(fr30_sub(a, b), one) and the verdict d == 0; variant 1 tests the difference as it is
Fr30 difference(Sum which, const Fr30& a, const Fr30& b, const Fr30& one, bool* zero) {
    const Fr30 raw = add(which, a, b, -1), d = mul(raw, one);
    if (variant == 1) {
        uint32_t l[8];
        to_limbs(raw, l);
        *zero = all_zero(l);
    } else {
        *zero = cvb_is_zero(d);
    }
    return d;
}

// glv_split_device, the loop as the unit states it (tests/test_cvb_extremes.py holds this text to the unit's)
constexpr uint64_t kLambdaHi = 0xac45a4010001a402ULL, kLambdaLo = 0x00000000ffffffffULL;
void glv_split(const uint32_t l[8], uint64_t k1[2], uint64_t k2[2]) {
    uint64_t v0 = l[0] | ((uint64_t)l[1] << 32), v1 = l[2] | ((uint64_t)l[3] << 32), v2 = l[4] | ((uint64_t)l[5] << 32),
             v3 = l[6] | ((uint64_t)l[7] << 32);
    uint64_t r0 = 0, r1 = 0, q0 = 0, q1 = 0;
    for (int bit = 0; bit < 256; bit++) {
        const bool over = (r1 >> 63) != 0;  // the remainder shifted left passes 2^128: it is above lambda then
        r1 = (r1 << 1) | (r0 >> 63);
        r0 = (r0 << 1) | (v3 >> 63);
        v3 = (v3 << 1) | (v2 >> 63);
        v2 = (v2 << 1) | (v1 >> 63);
        v1 = (v1 << 1) | (v0 >> 63);
        v0 <<= 1;
        q1 = (q1 << 1) | (q0 >> 63);
        q0 <<= 1;
        if (over || r1 > kLambdaHi || (r1 == kLambdaHi && r0 >= kLambdaLo)) {
            const uint64_t borrow = r0 < kLambdaLo ? 1 : 0;
            r0 -= kLambdaLo;
            r1 = r1 - kLambdaHi - borrow;
            q0 |= 1;
        }
    }
    k1[0] = r0;
    k1[1] = r1;
    k2[0] = q0;
    k2[1] = q1;
}

bool hex_limbs(const char* h, uint32_t l[8]) {
    if (strlen(h) != 64) return false;
    for (int w = 0; w < 8; w++) {
        uint32_t v = 0;
        for (int c = 0; c < 8; c++) {
            const char ch = h[(7 - w) * 8 + c];
            const int d = ch >= '0' && ch <= '9' ? ch - '0' : (ch >= 'a' && ch <= 'f' ? ch - 'a' + 10 : -1);
            if (d < 0) return false;
            v = (v << 4) | (uint32_t)d;
        }
        l[w] = v;
    }
    return true;
}
bool ok = true;
kzg_host::Fr read_fr() {
    char h[80];
    uint32_t l[8] = {};
    ok = ok && scanf("%79s", h) == 1 && hex_limbs(h, l);
    kzg_host::Fr w;
    memcpy(w.l, l, 32);
    return w;
}
Fr30 read_multiplier() {
    const Fr30 v = fr30_arg_from_mont256(read_fr());
    digits(v, -1);
    return v;
}
kzg_host::Fr pow2(int k) {
    kzg_host::Fr v = kzg_host::kFrOne;
    for (int i = 0; i < k; i++) v = kzg_host::fr_add(v, v);
    return v;
}
Fr30 k284, one;
// cvb_ld_m: a blst_fr image into the multiplier form
Fr30 ld_m(const kzg_host::Fr& w) {
    uint32_t l[8];
    memcpy(l, w.l, 32);
    const Fr30 v = fr30_from_limbs(l);
    digits(v, -1);
    return mul(v, k284);
}
void print_limbs(const uint32_t l[8]) {
    for (int w = 7; w >= 0; w--) printf("%08x", l[w]);
}

constexpr int kLanes = 64, kMaxT = 7, kMaxG = 8;

// cvb_group_inverse for the 64 lanes of a workgroup
void group_inverse(const Fr30* d, Fr30* out) {
    Fr30 mp[kLanes], ms[kLanes], p[kLanes], s[kLanes];
    for (int t = 0; t < kLanes; t++) mp[t] = ms[t] = d[t];
    for (int o = 1; o < kLanes; o <<= 1) {
        for (int t = 0; t < kLanes; t++) {
            p[t] = mp[t];
            s[t] = ms[t];
        }
        for (int t = 0; t < kLanes; t++) {
            if (t >= o) mp[t] = mul(p[t - o], mp[t]);
            if (t + o < kLanes) ms[t] = mul(ms[t], s[t + o]);
        }
    }
    const Fr30 inv = fr30_inv(ms[0]);
    digits(inv, kProdTop);
    for (int t = 0; t < kLanes; t++) {
        Fr30 v = inv;
        if (t > 0) v = mul(v, mp[t - 1]);
        if (t + 1 < kLanes) v = mul(v, ms[t + 1]);
        out[t] = v;
    }
}

// k_cvb_public: one workgroup
Fr30 public_at(const Fr30& z, const std::vector<kzg_host::Fr>& pub, const Fr30& w, const Fr30& w64, const Fr30& invn, int lg_n,
               long* hit_out) {
    const uint32_t n_public = (uint32_t)pub.size();
    uint32_t hit = 0xffffffffu;
    Fr30 wcur[kLanes], acc[kLanes], d[kLanes], dinv[kLanes];
    bool live[kLanes];
    for (uint32_t t = 0; t < kLanes; t++) {
        wcur[t] = one;
        Fr30 base = w;
        for (uint32_t bit = 0; bit < 6; bit++) {
            if ((t >> bit) & 1) wcur[t] = mul(wcur[t], base);
            base = mul(base, base);
        }
        acc[t] = fr30_zero();
    }
    for (uint32_t base = 0; base < n_public; base += kLanes) {
        for (uint32_t t = 0; t < kLanes; t++) {
            const uint32_t i = base + t;
            live[t] = i < n_public;
            d[t] = one;
            if (live[t]) {
                bool zero;
                d[t] = difference(kZw, z, wcur[t], one, &zero);
                if (zero) {
                    if (i < hit) hit = i;
                    d[t] = one;
                    live[t] = false;
                }
            }
        }
        group_inverse(d, dinv);
        for (uint32_t t = 0; t < kLanes; t++) {
            if (live[t]) acc[t] = mul(add(kAcc, acc[t], mul(mul(ld_m(pub[base + t]), wcur[t]), dinv[t])), one);
            wcur[t] = mul(wcur[t], w64);
        }
    }
    *hit_out = hit == 0xffffffffu ? -1 : (long)hit;
    if (hit != 0xffffffffu) return ld_m(pub[hit]);
    Fr30 total = acc[0];
    for (uint32_t q = 1; q < kLanes; q++) total = add(kTotal, total, acc[q]);
    Fr30 zn = z;
    for (int q = 0; q < lg_n; q++) zn = mul(zn, zn);
    return mul(mul(total, one), mul(add(kZn1, zn, one, -1), invn));
}

Fr30 cvb_pow(const Fr30& v, uint32_t n) {
    Fr30 p = one;
    for (uint32_t i = 0; i < n; i++) p = mul(p, v);
    return p;
}

}  // namespace

int main() {
    int t = 0, lg_n = 0, e = 0, g = 0, n_public = 0, count = 0;
    if (scanf("%d %d %d %d %d %d %d", &variant, &t, &lg_n, &e, &g, &n_public, &count) != 7 || variant < 0 || variant > 2 || t < 2 ||
        t > kMaxT || lg_n < 1 || lg_n > 32 || e < 1 || e > 8 || g < 0 || g > kMaxG || n_public < 0 || n_public > 4096 || count < 1 ||
        count > 4096)
        return 2;
    int exps[kMaxG * kMaxT] = {};
    for (int i = 0; i < g * t; i++)
        if (scanf("%d", &exps[i]) != 1 || exps[i] < 0 || exps[i] > 7) return 2;
    k284 = fr30_arg_from_mont256(pow2(14));
    one = fr30_const_one270();
    const Fr30 w = read_multiplier(), w1 = read_multiplier(), invn = read_multiplier(), w64 = read_multiplier();
    Fr30 shifts[kMaxT];
    for (int j = 0; j < t; j++) shifts[j] = read_multiplier();
    if (!ok) return 2;
    struct Line {
        char tag;
        uint32_t l[8];
        uint64_t k1[2], k2[2];
    };
    struct Out {
        uint32_t pi[8];
        long hit;
        uint32_t lin[4][8];
        std::vector<Line> q;
    };
    std::vector<Out> outs;
    for (int k = 0; k < count; k++) {
        kzg_host::Fr ch[6], ev[2 * kMaxT];
        for (int i = 0; i < 6; i++) ch[i] = read_fr();
        for (int i = 0; i < 2 * t; i++) ev[i] = read_fr();
        std::vector<kzg_host::Fr> pub(n_public);
        for (int i = 0; i < n_public; i++) pub[i] = read_fr();
        if (!ok) return 2;
        Out o;
        // ---- k_cvb_public ----
        Fr30 pim = fr30_zero();
        o.hit = -1;
        if (n_public) pim = public_at(ld_m(ch[3]), pub, w, w64, invn, lg_n, &o.hit);
        cvb_plain(pim, o.pi);
        // ---- k_cvb_lin ----
        Fr30 lin[4];
        {
            const Fr30 ze = ld_m(ch[3]);
            Fr30 zn = ze;
            for (int q = 0; q < lg_n; q++) zn = mul(zn, zn);
            bool is_one;
            Fr30 d = difference(kZn1, ze, one, one, &is_one);
            if (is_one) d = one;
            const Fr30 dinv = fr30_inv(d);
            digits(dinv, kProdTop);
            const Fr30 l0 = is_one ? one : mul(mul(add(kZn1, zn, one, -1), invn), dinv);
            const Fr30 be = ld_m(ch[0]), ga = ld_m(ch[1]), al = ld_m(ch[2]);
            Fr30 A = one, B = ld_m(ev[2 * t - 1]);
            for (int j = 0; j < t; j++) {
                const Fr30 ag = add(kAg, ld_m(ev[j]), ga);
                A = mul(A, add(kFactor, ag, mul(mul(be, shifts[j]), ze)));
                if (j + 1 < t) B = mul(B, add(kFactor, ag, mul(be, ld_m(ev[t + j]))));
            }
            const Fr30 a2l = mul(mul(al, al), l0), aB = mul(al, B);
            const Fr30 sc_z = add(kScZ, mul(al, A), a2l), sc_sig = neg(mul(aB, be));
            Fr30 konst = n_public ? pim : fr30_zero();
            konst = add(kKonst, add(kKonst, konst, mul(aB, add(kAg, ld_m(ev[t - 1]), ga)), -1), a2l, -1);
            lin[0] = zn;
            lin[1] = sc_z;
            lin[2] = sc_sig;
            lin[3] = konst;
            for (int i = 0; i < 4; i++) cvb_plain(lin[i], o.lin[i]);
        }
        // ---- k_cvb_scalars, lane q ----
        const uint32_t T = (uint32_t)t, nkey = 2 * T + 2 + (uint32_t)g, nk = nkey + 1, per = T + (uint32_t)e, Q = per + 5 + 2 * nk;
        for (uint32_t q = 0; q < Q; q++) {
            const Fr30 r = ld_m(ch[5]);
            Fr30 val = one, scale = r;
            bool split = true, v2 = false;
            if (q < T) {
                val = cvb_pow(ld_m(ch[4]), q + 1);
            } else if (q == T) {
                val = lin[1];
            } else if (q < per) {
                const Fr30 zn = lin[0];
                val = mul(neg(add(kZn1, zn, one, -1)), cvb_pow(zn, q - T - 1));
            } else if (q == per) {
                val = cvb_pow(ld_m(ch[4]), 2 * T);
            } else if (q < per + 5) {
                const uint32_t j = q - per - 1;
                const Fr30 ze = ld_m(ch[3]);
                const Fr30 mzw = neg(mul(ze, w));
                val = j == 0 ? mzw : (j == 1 ? neg(ze) : (j == 2 ? mul(mzw, ze) : mul(ze, w1)));
                scale = one;
            } else {
                const uint32_t jj = q - per - 5, j = jj < nk ? jj : jj - nk;
                const bool p0 = jj < nk;
                split = false;
                const Fr30 ze = ld_m(ch[3]);
                const Fr30 mzw = neg(mul(ze, w));
                if (p0) scale = mul(r, mzw);
                if (j < T) {
                    val = ld_m(ev[j]);
                } else if (j == T) {
                    val = mul(ld_m(ev[0]), ld_m(ev[1]));
                } else if (j == T + 1) {
                    val = one;
                } else if (j < 2 * T + 1) {
                    val = cvb_pow(ld_m(ch[4]), j - 1);
                } else if (j == 2 * T + 1) {
                    val = lin[2];
                } else if (j < nkey) {
                    const uint32_t sx = j - 2 * T - 2;
                    val = one;
                    for (uint32_t i = 0; i < T; i++) {
                        const Fr30 a = ld_m(ev[i]);
                        for (int c = 0; c < exps[sx * T + i]; c++) val = mul(val, a);
                    }
                } else {
                    const Fr30 v = ld_m(ch[4]);
                    Fr30 g0 = lin[3], vp = one;
                    for (uint32_t i = 1; i < 2 * T; i++) {
                        vp = mul(vp, v);
                        g0 = add(kG0, g0, mul(vp, ld_m(ev[i - 1])), -1);
                    }
                    const Fr30 g1 = neg(mul(mul(vp, v), ld_m(ev[2 * T - 1])));
                    if (p0) {
                        val = add(kG01, mul(mzw, g0), mul(neg(ze), g1));
                        scale = r;
                    } else {
                        val = add(kG01, g0, g1);
                        v2 = variant == 2;
                    }
                }
            }
            Line ln;
            ln.tag = split ? 's' : 'r';
            if (v2) {
                to_limbs(val, ln.l);
            } else {
                val = mul(scale, val);
                cvb_plain(val, ln.l);
            }
            if (split) glv_split(ln.l, ln.k1, ln.k2);
            o.q.push_back(ln);
        }
        outs.push_back(o);
    }
    printf("%d %d\n", kR9SumRawBound, kR9SumNormBound);
    for (int i = 0; i < kReports; i++) printf("%llu ", (unsigned long long)rep[i]);
    printf("%lld %lld %llu %llu %llu %lld\n", (long long)(lo_r * 1048576.0L), (long long)(hi_r * 1048576.0L), (unsigned long long)outside,
           (unsigned long long)at_minus_r, (unsigned long long)at_plus_r, (long long)(own_r * 1048576.0L) + 1);
    for (const Out& o : outs) {
        printf("pi ");
        print_limbs(o.pi);
        printf(" %ld\nlin", o.hit);
        for (int i = 0; i < 4; i++) {
            printf(" ");
            print_limbs(o.lin[i]);
        }
        printf("\n");
        for (const Line& ln : o.q) {
            printf("%c ", ln.tag);
            print_limbs(ln.l);
            if (ln.tag == 's')
                printf(" %016llx%016llx %016llx%016llx", (unsigned long long)ln.k1[1], (unsigned long long)ln.k1[0],
                       (unsigned long long)ln.k2[1], (unsigned long long)ln.k2[0]);
            printf("\n");
        }
    }
    return 0;
}
