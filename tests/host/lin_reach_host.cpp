// Host replay of k_lin_combine's accumulation (csrc/linearise_kernels.hip) on the unchanged csrc/fr30.hip.h, for
// tests/test_circuit_open.py: a stand-alone program (plain g++ -fwrapv; the header is __host__ __device__ code).  Test
// infrastructure only.
//
// It replays one index per input line in the kernel's order: the accumulator starts as the constant (a canonical value loaded like
// a coefficient), takes one product per column -- acc = norm(acc + c * mult / 2^270), fr30_mac -- and leaves through
// fr30_sum_reduce and fr30_to_limbs.  Not the memory layout, not the evaluation.
//
// stdin:   K C
//          K lines:  konst  mult_0 c_0  ..  mult_(C-1) c_(C-1)     (64 hex digits each: konst and c_k blst_fr images, mult_k the
//                                                                   image of the plain multiplier)
// stdout:  six numbers: the largest |digit 0..7| of a raw sum entering a carry pass, the largest |digit 0..7| leaving one (or a
//          load, or a product), the largest |digit 8| of an accumulator, the largest |digit 8| of a product, the largest |digit 8|
//          of what fr30_sum_reduce returns, the largest |column| of any product (exact, saturated at 2^64 - 1).  Then the K results.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../kzg_poly_commit_exploration_amd/csrc/fr30.hip.h"
#include "../../kzg_poly_commit_exploration_amd/csrc/host_fr.hpp"
#include "../../kzg_poly_commit_exploration_amd/csrc/fr30_host.hpp"

using namespace kzg;

namespace {

enum { kRaw = 0, kNorm, kAccTop, kProdTop, kReducedTop, kColumn, kReports };
uint64_t rep[kReports];
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
// fr30_mul with its columns followed in exact arithmetic; the product itself is the header's
Fr30 mul(const Fr30& a, const Fr30& b, int top) {
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
    digits(p, top);
    return p;
}
// fr30_mac: the raw digits reported in 64 bits, wrapped to 32 as the device would
Fr30 mac(const Fr30& acc, const Fr30& c, const Fr30& w) {
    const Fr30 p = mul(c, w, kProdTop);
    Fr30 r;
    for (int i = 0; i < kR9; i++) {
        const int64_t s = (int64_t)acc.d[i] + (int64_t)p.d[i];
        if (i < kR9 - 1) see(kRaw, s);
        r.d[i] = (int32_t)(uint32_t)(uint64_t)s;
    }
    r = fr30_norm(r);
    digits(r, kAccTop);
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
bool ok = true;
kzg_host::Fr read_fr() {
    char h[80];
    uint32_t l[8] = {};
    ok = ok && scanf("%79s", h) == 1 && hex_limbs(h, l);
    kzg_host::Fr w;
    memcpy(w.l, l, 32);
    return w;
}
Fr30 read_image() {
    const kzg_host::Fr w = read_fr();
    uint32_t l[8];
    memcpy(l, w.l, 32);
    const Fr30 v = fr30_from_limbs(l);
    digits(v, -1);
    return v;
}
void print(const Fr30& v) {
    uint32_t l[8];
    fr30_to_limbs(v, l);
    for (int w = 7; w >= 0; w--) printf("%08x", l[w]);
    printf("\n");
}

}  // namespace

int main() {
    int K = 0, C = 0;
    if (scanf("%d %d", &K, &C) != 2 || K < 1 || K > 4096 || C < 1 || C > 32) return 2;
    std::vector<Fr30> out;
    for (int k = 0; k < K; k++) {
        Fr30 acc = read_image();  // the constant, as the kernel loads it at index 0
        for (int j = 0; j < C; j++) {
            const Fr30 w = fr30_arg_from_mont256(read_fr());
            digits(w, -1);
            const Fr30 c = read_image();
            if (!ok) return 2;
            acc = mac(acc, c, w);
        }
        out.push_back(mul(acc, fr30_const_one270(), kReducedTop));  // fr30_sum_reduce
    }
    if (!ok) return 2;
    for (int i = 0; i < kReports; i++) printf("%llu%c", (unsigned long long)rep[i], i + 1 < kReports ? ' ' : '\n');
    for (const Fr30& v : out) print(v);
    return 0;
}
