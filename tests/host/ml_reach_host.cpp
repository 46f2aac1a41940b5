// Host replay of the multilinear kernels' arithmetic (csrc/multilinear_kernels.hip) on the unchanged csrc/fr30.hip.h, for
// tests/test_multilinear_reach.py: a stand-alone program (plain g++ -fwrapv; the header is __host__ __device__ code).  Test
// infrastructure only.
//
// It replays the order of products, sums and carry passes, not the memory layout:
//   fold     k_ml_fold's chain: K levels of a + u (b - a) over 2^K leaves, canonical after every fold (ml_fold1)
//   eval     k_ml_eval's accumulators: per lane the Horner chain of eight coefficients in z256, the product with the lane's power,
//            the sign of the odd lanes, and the sum of 256 lanes in cmb_workgroup_sum's order (eight pairwise levels, a carry pass
//            after every addition); then fr30_sum_reduce
//   combine  k_ml_combine's sum: a canonical start value and T - 1 products, a carry pass after each, then fr30_sum_reduce
//
// stdin:   "fold K L"     then L leaf images (cycled over the 2^K leaves), then K multipliers u_i (blst_fr images of the plain u_i)
//          "eval L"       then L coefficient images (lane t, step m takes number (t + 256 m) mod L), then z256 and zt (images of
//                         the plain multipliers; every lane uses zt)
//          "combine T L"  then L images (term i takes number i mod L), then T multipliers (the first is not used)
//          all numbers as 64 hex digits
// stdout:  four numbers: the largest |digit 0..7| of a raw sum or difference, the largest |digit 0..7| leaving a carry pass, a load
//          or a product, the largest |digit 8|, the largest |column| of any product (exact, saturated at 2^64 - 1); then the
//          results as images: fold -> v; eval -> the sum and the alternating sum; combine -> F
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../kzg_poly_commit_exploration_amd/csrc/fr30.hip.h"
#include "../../kzg_poly_commit_exploration_amd/csrc/host_fr.hpp"
#include "../../kzg_poly_commit_exploration_amd/csrc/fr30_host.hpp"

using namespace kzg;

namespace {

uint64_t rep[4];
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
// a + sign b digit-wise, raw: the digits reported in 64 bits, wrapped to 32 as the device would
Fr30 add_raw(const Fr30& a, const Fr30& b, int sign = 1) {
    Fr30 r;
    for (int i = 0; i < kR9; i++) {
        const int64_t s = (int64_t)a.d[i] + sign * (int64_t)b.d[i];
        see(i < kR9 - 1 ? 0 : 2, s);
        r.d[i] = (int32_t)(uint32_t)(uint64_t)s;
    }
    return r;
}
Fr30 norm(const Fr30& a) {
    const Fr30 r = fr30_norm(a);
    digits(r, 1);
    return r;
}
struct Limbs {
    uint32_t l[8];
};
Limbs read_image() {
    char buf[80];
    Limbs v;
    if (scanf("%79s", buf) != 1 || strlen(buf) != 64) {
        fprintf(stderr, "ml_reach: expected 64 hex digits\n");
        exit(2);
    }
    for (int w = 0; w < 8; w++) {
        char part[9];
        memcpy(part, buf + 8 * (7 - w), 8);
        part[8] = 0;
        v.l[w] = (uint32_t)strtoul(part, nullptr, 16);
    }
    return v;
}
Fr30 read_multiplier() {  // the image of a plain multiplier -> the x 2^270 form, as the host path prepares it
    const Limbs v = read_image();
    kzg_host::Fr f;
    for (int i = 0; i < 4; i++) f.l[i] = (uint64_t)v.l[2 * i] | ((uint64_t)v.l[2 * i + 1] << 32);
    const Fr30 d = fr30_arg_from_mont256(f);
    digits(d, 1);
    return d;
}
Fr30 load(const Limbs& v) {
    const Fr30 d = fr30_from_limbs(v.l);
    digits(d, 1);
    return d;
}
std::vector<std::string> results;  // printed after the report, which the last reductions still feed
void print_image(const uint32_t l[8]) {
    char buf[72];
    for (int w = 7; w >= 0; w--) snprintf(buf + 8 * (7 - w), 9, "%08x", l[w]);
    results.push_back(buf);
}
void print_all() {
    printf("%llu %llu %llu %llu\n", (unsigned long long)rep[0], (unsigned long long)rep[1], (unsigned long long)rep[2],
           (unsigned long long)rep[3]);
    for (const auto& r : results) printf("%s\n", r.c_str());
}
// ml_fold1 of the kernel unit
Limbs fold1(const Limbs& a, const Limbs& b, const Fr30& u) {
    const Fr30 fa = load(a), fb = load(b);
    const Fr30 d = add_raw(fb, fa, -1);
    const Fr30 s = add_raw(fa, mul(u, d));
    Limbs o;
    fr30_to_limbs(s, o.l);
    return o;
}
void canonical_out(const Fr30& acc) {
    const Fr30 red = mul(acc, fr30_const_one270());  // fr30_sum_reduce
    uint32_t l[8];
    fr30_to_limbs(red, l);
    print_image(l);
}

}  // namespace

int main() {
    char mode[16];
    if (scanf("%15s", mode) != 1) return 2;
    if (!strcmp(mode, "fold")) {
        int K, L;
        if (scanf("%d %d", &K, &L) != 2 || K < 1 || K > 16 || L < 1) return 2;
        std::vector<Limbs> in(L), cur((size_t)1 << K);
        for (auto& v : in) v = read_image();
        for (size_t j = 0; j < cur.size(); j++) cur[j] = in[j % L];
        for (int i = 0; i < K; i++) {
            const Fr30 u = read_multiplier();
            for (size_t j = 0; j < cur.size() / 2; j++) cur[j] = fold1(cur[2 * j], cur[2 * j + 1], u);
            cur.resize(cur.size() / 2);
        }
        print_image(cur[0].l);
    } else if (!strcmp(mode, "eval")) {
        int L;
        if (scanf("%d", &L) != 1 || L < 1) return 2;
        std::vector<Limbs> in(L);
        for (auto& v : in) v = read_image();
        const Fr30 z256 = read_multiplier(), zt = read_multiplier();
        std::vector<Fr30> a(256), b(256);
        for (int t = 0; t < 256; t++) {
            Fr30 h = fr30_zero();
            for (int m = 7; m >= 0; m--) h = add_raw(mul(h, z256), load(in[(t + 256 * m) % L]));
            a[t] = mul(h, zt);
            for (int k = 0; k < kR9; k++) b[t].d[k] = (t & 1) ? -a[t].d[k] : a[t].d[k];
        }
        for (int w = 1; w < 256; w *= 2)  // the eight pairwise levels of cmb_workgroup_sum, a carry pass after every addition
            for (int t = 0; t < 256; t += 2 * w) {
                a[t] = norm(add_raw(a[t], a[t + w]));
                b[t] = norm(add_raw(b[t], b[t + w]));
            }
        canonical_out(a[0]);
        canonical_out(b[0]);
    } else if (!strcmp(mode, "combine")) {
        int T, L;
        if (scanf("%d %d", &T, &L) != 2 || T < 1 || T > 64 || L < 1) return 2;
        std::vector<Limbs> in(L);
        for (auto& v : in) v = read_image();
        Fr30 acc = load(in[0]);
        for (int i = 0; i < T; i++) {
            const Fr30 g = read_multiplier();
            if (i == 0) continue;
            acc = norm(add_raw(acc, mul(load(in[i % L]), g)));  // fr30_mac
        }
        canonical_out(acc);
    } else {
        return 2;
    }
    print_all();
    return 0;
}
