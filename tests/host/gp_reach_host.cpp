// Host replay of the grand-product kernels' arithmetic (csrc/grand_product_kernels.hip) on the unchanged csrc/fr30.hip.h, for
// tests/test_grand_product.py: a stand-alone program (plain g++ -fwrapv; the header is __host__ __device__ code).  Test
// infrastructure only.
//
// It replays the per-element step of both forms (the products of the t factors, the product with 2^(270 + 14 t)), the products
// of a run of 4 and its v_i, the two Hillis-Steele scans over the 256 lanes of a tile, u_i, the carry kernel (runs of tiles, the same
// scans, the one inversion, c_T, last) and the scale pass -- the order of products, sums and carry passes, not the memory
// layout.  In the permutation form the twiddle w^i is an INPUT, so the test can make it extremal.
//
// stdin:   form t tiles K               (form 0: general, 1: permutation; n = tiles x 1024)
//          form 1 only: beta gamma bk_0 .. bk_(t-1)      (blst_fr images, 64 hex digits each; bk_j = beta k_j)
//          K lines, form 0:  a_0 .. a_(t-1) b_0 .. b_(t-1)            (images)
//                   form 1:  w f_0 .. f_(t-1) s_0 .. s_(t-1)          (w: the image of the plain twiddle; f, s: images)
//          index i uses line i mod K (K a divisor of 1024: tile 0 stands for all)
// stdout:  four numbers: the largest |digit 0..7| entering a carry pass as a raw sum, the largest |digit 0..7| leaving a carry
//          pass, a load or a product, the largest |digit 8|, the largest |column| of any product (exact, saturated at
//          2^64 - 1); then three counts: denominators b_j[i] of the permutation form whose sum was exactly 0, r, 2 r BEFORE any
//          reduction; then the least index with B_i = 0 or -1; then last; then z of the first K and of the last K indices.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../kzg_poly_commit_exploration_amd/csrc/fr30.hip.h"
#include "../../kzg_poly_commit_exploration_amd/csrc/host_fr.hpp"
#include "../../kzg_poly_commit_exploration_amd/csrc/fr30_host.hpp"

using namespace kzg;

namespace {

uint64_t rep[4];
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
// a + b digit-wise, carry-normalised: the raw digits reported in 64 bits, wrapped to 32 as the device would
Fr30 add(const Fr30& a, const Fr30& b) {
    Fr30 r;
    for (int i = 0; i < kR9; i++) {
        const int64_t s = (int64_t)a.d[i] + (int64_t)b.d[i];
        see(i < kR9 - 1 ? 0 : 2, s);
        r.d[i] = (int32_t)(uint32_t)(uint64_t)s;
    }
    r = fr30_norm(r);
    digits(r, 1);
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
Fr30 read_multiplier() {
    char h[80];
    uint32_t l[8] = {};
    ok = ok && scanf("%79s", h) == 1 && hex_limbs(h, l);
    kzg_host::Fr w;
    memcpy(w.l, l, 32);
    return fr30_arg_from_mont256(w);
}
void print(const Fr30& v) {
    uint32_t l[8];
    fr30_to_limbs(v, l);
    for (int w = 7; w >= 0; w--) printf("%08x", l[w]);
    printf("\n");
}
bool is_zero(const Fr30& v) {
    uint32_t l[8];
    fr30_to_limbs(v, l);
    return (l[0] | l[1] | l[2] | l[3] | l[4] | l[5] | l[6] | l[7]) == 0;
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

constexpr int kMaxT = 16;
struct Line {
    Fr30 w;                      // form 1: the twiddle, a multiplier
    Fr30 a[kMaxT], b[kMaxT];     // form 0: the factors; form 1: f_j and s_j
};
struct Perm {
    Fr30 beta, gamma, bk[kMaxT];
};

// A_i and B_i in multiplier form, as gp_element and the product with `scale` form them
void element(int form, int t, const Line& e, const Perm& pm, const Fr30& scale, Fr30& A, Fr30& B) {
    Fr30 a, b;
    if (form == 0) {
        a = e.a[0];
        b = e.b[0];
        for (int j = 1; j < t; j++) {
            a = mul(a, e.a[j]);
            b = mul(b, e.b[j]);
        }
    } else {
        for (int j = 0; j < t; j++) {
            const Fr30 fg = add(e.a[j], pm.gamma);
            const Fr30 aj = add(fg, mul(pm.bk[j], e.w));
            const Fr30 bj = add(fg, mul(e.b[j], pm.beta));
            const int k = multiple_of_r(bj);
            if (k >= 0) zsum[k]++;
            a = j ? mul(a, aj) : aj;
            b = j ? mul(b, bj) : bj;
        }
    }
    A = mul(a, scale);
    B = mul(b, scale);
}
// fr30_scan_products (fr30_lanes.hip.h) over 256 lanes: inclusive prefix of p, inclusive suffix of s, with the kernel's operand order
void scan(std::vector<Fr30>& p, std::vector<Fr30>& s) {
    for (int o = 1; o < 256; o <<= 1) {
        const std::vector<Fr30> p0 = p, s0 = s;
        for (int t = 0; t < 256; t++) {
            if (t >= o) p[t] = mul(p0[t - o], p0[t]);
            if (t + o < 256) s[t] = mul(s0[t], s0[t + o]);
        }
    }
}

}  // namespace

int main() {
    int form = 0, t = 0, tiles = 0, K = 0;
    if (scanf("%d %d %d %d", &form, &t, &tiles, &K) != 4 || form < 0 || form > 1 || t < 1 || t > kMaxT || tiles < 1 || tiles > 4096 ||
        K < 1 || K > 1024 || 1024 % K)
        return 2;
    Perm pm{};
    if (form == 1) {
        pm.beta = read_multiplier();
        pm.gamma = read_image();
        for (int j = 0; j < t; j++) pm.bk[j] = read_image();
    }
    std::vector<Line> el(K);
    for (int k = 0; k < K; k++) {
        if (form == 1) el[k].w = read_multiplier();
        for (int j = 0; j < t; j++) el[k].a[j] = read_image();
        for (int j = 0; j < t; j++) el[k].b[j] = read_image();
    }
    if (!ok) return 2;
    kzg_host::Fr p2 = kzg_host::kFrOne;
    for (int i = 0; i < 14 * t; i++) p2 = kzg_host::fr_add(p2, p2);
    const Fr30 scale = fr30_arg_from_mont256(p2), one = fr30_const_one270();
    uint32_t l1[8];
    memcpy(l1, kzg_host::kFrOne.l, 32);
    const Fr30 img_one = fr30_from_limbs(l1);

    // k_gp_tile on tile 0 (every tile sees the same elements)
    long bad = -1;
    std::vector<Fr30> u(1024), lane_a(256), lane_b(256);
    std::vector<Fr30> pa(1024), sb(1024);
    for (int lane = 0; lane < 256; lane++) {
        for (int k = 0; k < 4; k++) {
            const int i = 4 * lane + k;
            Fr30 A, B;
            element(form, t, el[i % K], pm, scale, A, B);
            if (is_zero(B) && bad < 0) bad = i;
            pa[i] = k ? mul(pa[i - 1], A) : A;
            sb[i] = B;
        }
        for (int k = 2; k >= 0; k--) sb[4 * lane + k] = mul(sb[4 * lane + k], sb[4 * lane + k + 1]);
        lane_a[lane] = pa[4 * lane + 3];
        lane_b[lane] = sb[4 * lane];
        for (int k = 1; k < 4; k++) sb[4 * lane + k] = mul(pa[4 * lane + k - 1], sb[4 * lane + k]);  // v_k: what the run knows of u_i
    }
    scan(lane_a, lane_b);
    for (int lane = 0; lane < 256; lane++) {
        Fr30 m = lane ? lane_a[lane - 1] : one;
        if (lane < 255) m = mul(m, lane_b[lane + 1]);
        for (int k = 0; k < 4; k++) u[4 * lane + k] = mul(sb[4 * lane + k], m);
    }
    const Fr30 tile_a = lane_a[255], tile_b = lane_b[0];

    // k_gp_carry
    const int run = (tiles + 255) / 256;
    std::vector<Fr30> ca(256), cb(256), c(tiles);
    for (int lane = 0; lane < 256; lane++) {
        Fr30 a = one, b = one;
        for (int k = lane * run; k < tiles && k < (lane + 1) * run; k++) {
            a = mul(a, tile_a);
            b = mul(b, tile_b);
        }
        ca[lane] = a;
        cb[lane] = b;
    }
    scan(ca, cb);
    const Fr30 binv = mul(inv(cb[0]), img_one);
    const Fr30 last = mul(ca[255], binv);
    for (int lane = 0; lane < 256; lane++) {
        const int first = lane * run < tiles ? lane * run : tiles, end = first + run < tiles ? first + run : tiles;
        Fr30 p = lane ? mul(ca[lane - 1], binv) : binv;
        for (int k = first; k < end; k++) {
            c[k] = p;
            p = mul(p, tile_a);
        }
        Fr30 s = lane < 255 ? cb[lane + 1] : one;
        for (int k = end; k > first; k--) {
            c[k - 1] = mul(c[k - 1], s);
            s = mul(s, tile_b);
        }
    }
    // k_gp_scale: u_i is stored canonical and loaded again
    auto z = [&](int tile, int i) {
        uint32_t l[8];
        fr30_to_limbs(u[i], l);
        const Fr30 v = fr30_from_limbs(l);
        digits(v, 1);
        return mul(v, c[tile]);
    };
    std::vector<Fr30> out;
    for (int k = 0; k < K; k++) out.push_back(z(0, k));
    for (int k = 0; k < K; k++) out.push_back(z(tiles - 1, 1024 - K + k));
    printf("%llu %llu %llu %llu\n", (unsigned long long)rep[0], (unsigned long long)rep[1], (unsigned long long)rep[2],
           (unsigned long long)rep[3]);
    printf("%ld %ld %ld\n%ld\n", zsum[0], zsum[1], zsum[2], bad);
    print(last);
    for (const Fr30& v : out) print(v);
    return 0;
}
