// Host replay of the evaluation-form quotient kernels' arithmetic (csrc/lagrange_kernels.hip) on the unchanged csrc/fr30.hip.h,
// for tests/test_lagrange.py: a stand-alone program (plain g++ -fwrapv; the header is __host__ __device__ code).  Test
// infrastructure only.
//
// It replays the per-element step of k_lagrange_partial's way back and the sums of a run, a tile and k_lagrange_finish -- the
// order of products, differences, carry passes and reductions, not the memory layout, the product scan or the inversion: the
// multipliers w^i and 1 / (z - w^i) are INPUTS, so the test can make them extremal.
//
// stdin:   tiles K y          (y: the claimed value, a blst_fr image as 64 hex digits)
//          K lines  f w dinv  (f: an image; w, dinv: the blst_fr images of the two multipliers; hex)
//          element i of the tiles x 1024 uses line i mod K (K a divisor of 1024: tile 0 stands for all); f_0 is line 0's f
// stdout:  four numbers: the largest |digit 0..7| entering a carry pass as a raw sum or difference, the largest |digit 0..7|
//          leaving a carry pass, a load or a product, the largest |digit 8|, the largest |column| of any product (exact,
//          saturated at 2^64 - 1); then the canonical sums sum f w dinv and sum q w; then "differs" 0 / 1; then K lines: q of
//          the first K elements.
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
// a + sign b digit-wise, carry-normalised: the raw digits reported in 64 bits, wrapped to 32 as the device would
Fr30 add(const Fr30& a, const Fr30& b, int sign = 1) {
    Fr30 r;
    for (int i = 0; i < kR9; i++) {
        const int64_t s = (int64_t)a.d[i] + sign * (int64_t)b.d[i];
        see(i < kR9 - 1 ? 0 : 2, s);
        r.d[i] = (int32_t)(uint32_t)(uint64_t)s;
    }
    r = fr30_norm(r);
    digits(r, 1);
    return r;
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
Fr30 load(const char* h, bool* ok) {
    uint32_t l[8] = {};
    *ok = *ok && hex_limbs(h, l);
    const Fr30 v = fr30_from_limbs(l);
    digits(v, 1);
    return v;
}
Fr30 mult(const char* h, bool* ok) {
    uint32_t l[8] = {};
    *ok = *ok && hex_limbs(h, l);
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
struct Element {
    Fr30 f, w, dinv;
};
struct Acc {
    Fr30 bary, dom;
};

}  // namespace

int main() {
    int tiles = 0, K = 0;
    char hy[80], hf[80], hw[80], hd[80];
    if (scanf("%d %d %79s", &tiles, &K, hy) != 3 || tiles < 1 || tiles > 4096 || K < 1 || K > 4096) return 2;
    bool ok = true;
    const Fr30 y = load(hy, &ok);
    std::vector<Element> el(K);
    for (int k = 0; k < K; k++) {
        if (scanf("%79s %79s %79s", hf, hw, hd) != 3) return 2;
        el[k] = Element{load(hf, &ok), mult(hw, &ok), mult(hd, &ok)};
    }
    if (!ok) return 2;
    const Fr30 one = fr30_const_one270(), f0 = el[0].f;
    std::vector<Fr30> q(K);
    std::vector<Acc> partial(tiles);
    bool differs = false;
    for (int tile = 0; tile < tiles; tile++) {
        if (tile > 0 && 1024 % K == 0) {  // every tile sees the same elements: the same record, computed once
            partial[tile] = partial[0];
            continue;
        }
        static Acc red[256];
        for (int t = 0; t < 256; t++) {
            Acc acc{fr30_zero(), fr30_zero()};
            for (int j = 3; j >= 0; j--) {  // lag_backward: the run from its last index down
                const size_t i = (size_t)tile * 1024 + j * 256 + t;
                const Element& e = el[i % K];
                if (!is_zero(add(e.f, f0, -1))) differs = true;
                const Fr30 qi = mul(add(y, e.f, -1), e.dinv);
                acc.bary = add(acc.bary, mul(mul(e.f, e.w), e.dinv));
                acc.dom = add(acc.dom, mul(qi, e.w));
                if (i < (size_t)K) q[i] = qi;
            }
            red[t] = Acc{mul(acc.bary, one), mul(acc.dom, one)};
        }
        for (int o = 128; o > 0; o >>= 1)
            for (int t = 0; t < o; t++) red[t] = Acc{add(red[t].bary, red[t + o].bary), add(red[t].dom, red[t + o].dom)};
        partial[tile] = Acc{mul(red[0].bary, one), mul(red[0].dom, one)};
    }
    Acc lanes[64];
    for (int l = 0; l < 64; l++) {  // k_lagrange_finish: lane l adds the tiles l + 64 k, lane 0 adds the 64 lanes
        lanes[l] = Acc{fr30_zero(), fr30_zero()};
        for (int k = l; k < tiles; k += 64) lanes[l] = Acc{add(lanes[l].bary, partial[k].bary), add(lanes[l].dom, partial[k].dom)};
    }
    Acc acc = lanes[0];
    for (int l = 1; l < 64; l++) acc = Acc{add(acc.bary, lanes[l].bary), add(acc.dom, lanes[l].dom)};
    const Fr30 bary = mul(acc.bary, one), dom = mul(acc.dom, one);
    printf("%llu %llu %llu %llu\n", (unsigned long long)rep[0], (unsigned long long)rep[1], (unsigned long long)rep[2],
           (unsigned long long)rep[3]);
    print(bary);
    print(dom);
    printf("%d\n", differs ? 1 : 0);
    for (int k = 0; k < K; k++) print(q[k]);
    return 0;
}
