// Host replay of the log-derivative kernels' arithmetic (csrc/lookup_kernels.hip) on the unchanged csrc/fr30.hip.h, for
// tests/test_lookup.py: a stand-alone program (plain g++ -fwrapv; the header is __host__ __device__ code).  Test infrastructure
// only.
//
// It replays the fraction recurrence of the general and the lookup form with the product by 2^(270 + 14 t), the run of 2, the two
// Hillis-Steele product scans and the additive scan over the 256 lanes of a tile, s_i and W_T, the carry kernel (runs of tiles, the
// same scans, the one inversion, c_T, the sums of c_T W_T, base_T, last) and the finish pass -- the order of products, sums and
// carry passes, not the memory layout -- and the count-to-image step of the multiplicities.
//
// stdin:   form t tiles K inject        (form 0: general, 1: lookup with k = t - 1 lookup columns, 2: counts; n = tiles x 512)
//          ext                          (an image; inject 1 / 2: EVERY term of the additive scans -- w_i in the tile, c_T W_T and the
//                                        reduced lane sums in the carry kernel -- is replaced by +ext / -ext where it is accumulated:
//                                        the sign-aligned extreme that inputs cannot force.  The sums then mean nothing: only the
//                                        report counts)
//          form 1 only: beta            (image)
//          K lines, form 0:  a_0 .. a_(t-1) b_0 .. b_(t-1)     (images)
//                   form 1:  f_0 .. f_(k-1) T m                (images)
//                   form 2:  one decimal count per line
//          row i uses line i mod K (K a divisor of 512: tile 0 stands for all)
// stdout:  five numbers: the largest |digit 0..7| entering a carry pass or a store as a raw sum, the largest |digit 0..7| leaving a
//          carry pass, a load or a product, the largest |digit 8|, the largest |column| of any product (exact, saturated at
//          2^64 - 1), the number of values outside (-r, 2 r) that went through fr30_to_limbs; then three counts: denominators
//          beta + f, beta + T of the lookup form whose sum was exactly 0, r, 2 r BEFORE any reduction; then the least row with
//          D_i = 0 or -1; then last; then phi of the first K and of the last K rows.  Form 2: the image of every count.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../kzg_poly_commit_exploration_amd/csrc/fr30.hip.h"
#include "../../kzg_poly_commit_exploration_amd/csrc/host_fr.hpp"
#include "../../kzg_poly_commit_exploration_amd/csrc/fr30_host.hpp"

using namespace kzg;

namespace {

uint64_t rep[5];
long zsum[3];
void see(int which, int64_t v) {
    const uint64_t m = v < 0 ? (uint64_t)(-v) : (uint64_t)v;
    if (m > rep[which]) rep[which] = m;
}
void digits(const Fr30& v, int which) {
    for (int i = 0; i < kR9 - 1; i++) see(which, v.d[i]);
    see(2, v.d[kR9 - 1]);
}
void column(__int128 acc) {
    const __int128 m = acc < 0 ? -acc : acc;
    const uint64_t s = m > (__int128)UINT64_MAX ? UINT64_MAX : (uint64_t)m;
    if (s > rep[3]) rep[3] = s;
}
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
    digits(p, 1);
    return p;
}
Fr30 sum_reduce(const Fr30& a) { return mul(a, fr30_const_one270()); }
// a + b digit-wise: the raw digits reported in 64 bits, wrapped to 32 as the device would
Fr30 add_raw(const Fr30& a, const Fr30& b) {
    Fr30 r;
    for (int i = 0; i < kR9; i++) {
        const int64_t s = (int64_t)a.d[i] + (int64_t)b.d[i];
        see(i < kR9 - 1 ? 0 : 2, s);
        r.d[i] = (int32_t)(uint32_t)(uint64_t)s;
    }
    return r;
}
Fr30 add(const Fr30& a, const Fr30& b) {
    const Fr30 r = fr30_norm(add_raw(a, b));
    digits(r, 1);
    return r;
}
Fr30 neg(const Fr30& a) {
    Fr30 r;
    for (int i = 0; i < kR9; i++) r.d[i] = -a.d[i];
    return r;
}
// fr30_inv with every product followed
Fr30 inv(const Fr30& a) {
    const uint64_t E[4] = {0xfffffffeffffffffULL, 0x53bda402fffe5bfeULL, 0x3339d80809a1d805ULL, 0x73eda753299d7d48ULL};  // r - 2
    const Fr30 a2 = mul(a, a), a3 = mul(a2, a);
    Fr30 acc = a;
    for (int w = 126; w >= 0; w--) {
        acc = mul(acc, acc);
        acc = mul(acc, acc);
        const uint32_t dgt = (uint32_t)(E[w >> 5] >> (2 * (w & 31))) & 3u;
        if (dgt) acc = mul(acc, dgt == 1 ? a : (dgt == 2 ? a2 : a3));
    }
    return acc;
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
Fr30 read_image() {
    char h[80];
    uint32_t l[8] = {};
    ok = ok && scanf("%79s", h) == 1 && hex_limbs(h, l);
    const Fr30 v = fr30_from_limbs(l);
    digits(v, 1);
    return v;
}
// k when the integer the digits stand for is exactly k r, k = 0, 1, 2; else -1
int multiple_of_r(const Fr30& v) {
    int64_t u[kR9], c = 0;
    for (int i = 0; i < kR9 - 1; i++) {
        const int64_t t = v.d[i] + c;
        u[i] = t & kR9Mask;
        c = t >> kR9Bits;
    }
    u[kR9 - 1] = v.d[kR9 - 1] + c;
    for (int k = 0; k < 3; k++) {
        int64_t carry = 0;
        bool same = true;
        for (int i = 0; i < kR9; i++) {
            const int64_t t = (int64_t)k * fr30_ru(i) + carry;
            const int64_t want = i < kR9 - 1 ? (t & kR9Mask) : t;
            carry = t >> kR9Bits;
            same = same && want == u[i];
        }
        if (same) return k;
    }
    return -1;
}
// fr30_to_limbs, with the check that the value lay in (-r, 2 r): v - canonical(v) + r is then 0, r or 2 r
Fr30 store(const Fr30& v) {
    uint32_t l[8];
    fr30_to_limbs(v, l);
    const Fr30 c = fr30_from_limbs(l);
    Fr30 d;
    for (int i = 0; i < kR9; i++) d.d[i] = v.d[i] - c.d[i] + fr30_rd(i);
    if (multiple_of_r(d) < 0) rep[4]++;
    digits(c, 1);
    return c;
}
void print(const Fr30& canonical) {
    uint32_t l[8];
    fr30_to_limbs(canonical, l);
    for (int w = 7; w >= 0; w--) printf("%08x", l[w]);
    printf("\n");
}
bool is_zero(const Fr30& v) {
    uint32_t l[8];
    fr30_to_limbs(v, l);
    return (l[0] | l[1] | l[2] | l[3] | l[4] | l[5] | l[6] | l[7]) == 0;
}

constexpr int kMaxT = 16, kTile = 512, kLanes = 256;
struct Line {
    Fr30 a[kMaxT], b[kMaxT];  // form 0: the columns; form 1: a[0 .. k-1] = f_j, b[0] = T, b[1] = m
};

// N_i and D_i in multiplier form, as lu_element and lu_row form them
void element(int form, int t, const Line& e, const Fr30& beta, const Fr30& img_one, const Fr30& scale, Fr30& N, Fr30& D) {
    auto den = [&](const Fr30& f) {
        const Fr30 b = add(f, beta);
        const int k = multiple_of_r(b);
        if (k >= 0) zsum[k]++;
        return b;
    };
    if (form == 0) {
        N = e.a[0];
        D = e.b[0];
        for (int j = 1; j < t; j++) {
            N = add(mul(N, e.b[j]), mul(e.a[j], D));
            D = mul(D, e.b[j]);
        }
    } else {
        D = den(e.a[0]);
        N = img_one;
        for (int j = 1; j + 1 < t; j++) {
            const Fr30 b = den(e.a[j]);
            N = add(mul(N, b), mul(img_one, D));
            D = mul(D, b);
        }
        const Fr30 b = den(e.b[0]);
        const Fr30 a = neg(e.b[1]);
        N = add(mul(N, b), mul(a, D));
        D = mul(D, b);
    }
    N = mul(N, scale);
    D = mul(D, scale);
}
// fr30_scan_products (fr30_lanes.hip.h) over 256 lanes: inclusive prefix of p, inclusive suffix of s, with the kernel's operand order
void scan(std::vector<Fr30>& p, std::vector<Fr30>& s) {
    for (int o = 1; o < kLanes; o <<= 1) {
        const std::vector<Fr30> p0 = p, s0 = s;
        for (int t = 0; t < kLanes; t++) {
            if (t >= o) p[t] = mul(p0[t - o], p0[t]);
            if (t + o < kLanes) s[t] = mul(s0[t], s0[t + o]);
        }
    }
}
// lu_scan_add: inclusive sums
void scan_add(std::vector<Fr30>& a) {
    for (int o = 1; o < kLanes; o <<= 1) {
        const std::vector<Fr30> a0 = a;
        for (int t = 0; t < kLanes; t++)
            if (t >= o) a[t] = add(a0[t - o], a0[t]);
    }
}

}  // namespace

int main() {
    int form = 0, t = 0, tiles = 0, K = 0, inject = 0;
    if (scanf("%d %d %d %d %d", &form, &t, &tiles, &K, &inject) != 5 || form < 0 || form > 2 || t < 1 || t > kMaxT || (form == 1 && t < 2) ||
        tiles < 1 || tiles > 8192 || K < 1 || K > kTile || (form != 2 && kTile % K) || inject < 0 || inject > 2)
        return 2;
    Fr30 ext = read_image();
    if (inject == 2) ext = neg(ext);
    if (form == 2) {  // k_lu_counts
        kzg_host::Fr p2 = kzg_host::kFrOne;
        for (int i = 0; i < 256; i++) p2 = kzg_host::fr_add(p2, p2);
        const Fr30 count_img = fr30_arg_from_mont256(p2);
        std::vector<Fr30> out;
        for (int k = 0; k < K; k++) {
            unsigned c = 0;
            if (scanf("%u", &c) != 1) return 2;
            const Fr30 d = fr30_small((int32_t)c);
            digits(d, 1);
            out.push_back(store(mul(d, count_img)));
        }
        printf("%llu %llu %llu %llu %llu\n", (unsigned long long)rep[0], (unsigned long long)rep[1], (unsigned long long)rep[2],
               (unsigned long long)rep[3], (unsigned long long)rep[4]);
        for (const Fr30& v : out) print(v);
        return 0;
    }
    Fr30 beta = fr30_zero();
    if (form == 1) beta = read_image();
    std::vector<Line> el(K);
    for (int k = 0; k < K; k++) {
        if (form == 0) {
            for (int j = 0; j < t; j++) el[k].a[j] = read_image();
            for (int j = 0; j < t; j++) el[k].b[j] = read_image();
        } else {
            for (int j = 0; j + 1 < t; j++) el[k].a[j] = read_image();
            el[k].b[0] = read_image();
            el[k].b[1] = read_image();
        }
    }
    if (!ok) return 2;
    kzg_host::Fr p2 = kzg_host::kFrOne;
    for (int i = 0; i < 14 * t; i++) p2 = kzg_host::fr_add(p2, p2);
    const Fr30 scale = fr30_arg_from_mont256(p2), one = fr30_const_one270(), zero = fr30_zero();
    uint32_t l1[8];
    memcpy(l1, kzg_host::kFrOne.l, 32);
    const Fr30 img_one = fr30_from_limbs(l1);

    // k_lu_tile on tile 0 (every tile sees the same rows)
    long bad = -1;
    std::vector<Fr30> N(kTile), D(kTile), s(kTile), lane_p(kLanes), lane_s(kLanes), lane_w(kLanes), w0(kLanes);
    for (int i = 0; i < kTile; i++) {
        element(form, t, el[i % K], beta, img_one, scale, N[i], D[i]);
        if (is_zero(D[i]) && bad < 0) bad = i;
    }
    for (int lane = 0; lane < kLanes; lane++) lane_p[lane] = lane_s[lane] = mul(D[2 * lane], D[2 * lane + 1]);
    scan(lane_p, lane_s);
    for (int lane = 0; lane < kLanes; lane++) {
        const Fr30 pl = lane ? lane_p[lane - 1] : one, sl = lane + 1 < kLanes ? lane_s[lane + 1] : one;
        const Fr30 u0 = mul(pl, mul(D[2 * lane + 1], sl)), u1 = mul(mul(pl, D[2 * lane]), sl);
        Fr30 a0 = mul(N[2 * lane], u0), a1 = mul(N[2 * lane + 1], u1);
        if (inject) a0 = a1 = ext;
        w0[lane] = a0;
        lane_w[lane] = add(a0, a1);
    }
    scan_add(lane_w);
    for (int lane = 0; lane < kLanes; lane++) {
        const Fr30 e = lane ? lane_w[lane - 1] : zero;
        s[2 * lane] = store(sum_reduce(e));
        s[2 * lane + 1] = store(sum_reduce(add(e, w0[lane])));
    }
    const Fr30 tile_d = lane_p[kLanes - 1], tile_w = sum_reduce(lane_w[kLanes - 1]);

    // k_lu_carry
    const int run = (tiles + kLanes - 1) / kLanes;
    std::vector<Fr30> cp(kLanes), cs(kLanes), c(tiles), base(tiles), tot(kLanes);
    for (int lane = 0; lane < kLanes; lane++) {
        Fr30 b = one;
        for (int k = lane * run; k < tiles && k < (lane + 1) * run; k++) b = mul(b, tile_d);
        cp[lane] = cs[lane] = b;
    }
    scan(cp, cs);
    const Fr30 dinv = mul(inv(cs[0]), img_one);
    auto term = [&](int k) { return inject ? ext : mul(c[k], tile_w); };
    for (int lane = 0; lane < kLanes; lane++) {
        const int first = lane * run < tiles ? lane * run : tiles, end = first + run < tiles ? first + run : tiles;
        Fr30 p = lane ? mul(cp[lane - 1], dinv) : dinv;
        for (int k = first; k < end; k++) {
            c[k] = p;
            p = mul(p, tile_d);
        }
        Fr30 sf = lane + 1 < kLanes ? cs[lane + 1] : one, sum = zero;
        for (int k = end; k > first; k--) {
            c[k - 1] = mul(c[k - 1], sf);
            sum = add(sum, term(k - 1));
            sf = mul(sf, tile_d);
        }
        tot[lane] = inject ? ext : sum_reduce(sum);
    }
    scan_add(tot);
    const Fr30 last = store(sum_reduce(tot[kLanes - 1]));
    for (int lane = 0; lane < kLanes; lane++) {
        const int first = lane * run < tiles ? lane * run : tiles, end = first + run < tiles ? first + run : tiles;
        Fr30 b = lane ? tot[lane - 1] : zero;
        for (int k = first; k < end; k++) {
            base[k] = store(sum_reduce(b));
            b = add(b, term(k));
        }
    }
    // k_lu_finish: s_i and base_T are stored canonical and loaded again
    auto phi = [&](int tile, int i) { return store(add_raw(mul(s[i], c[tile]), base[tile])); };
    std::vector<Fr30> out;
    for (int k = 0; k < K; k++) out.push_back(phi(0, k));
    for (int k = 0; k < K; k++) out.push_back(phi(tiles - 1, kTile - K + k));
    printf("%llu %llu %llu %llu %llu\n", (unsigned long long)rep[0], (unsigned long long)rep[1], (unsigned long long)rep[2],
           (unsigned long long)rep[3], (unsigned long long)rep[4]);
    printf("%ld %ld %ld\n%ld\n", zsum[0], zsum[1], zsum[2], bad);
    print(last);
    for (const Fr30& v : out) print(v);
    return 0;
}
