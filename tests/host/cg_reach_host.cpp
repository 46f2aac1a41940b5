// Host replay of k_cg_gate's arithmetic (csrc/custom_gate_kernels.hip) on the unchanged csrc/fr30.hip.h, for
// tests/test_circuit_custom.py: a stand-alone program (plain g++ -fwrapv; the header is __host__ __device__ code).  Test
// infrastructure only.
//
// It replays one coset point per input line in the kernel's order of products, sums and carry passes -- per term s: A = qx_s; per
// wire j with p[s][j] > 0: W = f_j k14, then A = A W p[s][j] times; S = S + A with one carry pass; G' = S x one -- not the memory
// layout.
//
// stdin:   K
//          K lines:  t g  p[0][0] .. p[g-1][t-1]  f_0 .. f_(t-1)  qx_0 .. qx_(g-1)      (blst_fr images, 64 hex digits each)
// stdout:  one line of reports, then per input line G' (a canonical image).  The reports: the largest |digit 0..7| entering the
//          sum's carry pass as a raw sum, the largest |digit 8| leaving it, the largest |digit 0..7| leaving any carry pass, load or
//          product, the largest |digit 8| of any product, the largest |column| of any product (exact, saturated at 2^64 - 1).
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../kzg_poly_commit_exploration_amd/csrc/fr30.hip.h"
#include "../../kzg_poly_commit_exploration_amd/csrc/host_fr.hpp"
#include "../../kzg_poly_commit_exploration_amd/csrc/fr30_host.hpp"

using namespace kzg;

namespace {

enum { kRaw = 0, kTop, kNorm, kProdTop, kColumn, kReports };
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
// fr30_mul with its columns followed in exact arithmetic; the product itself is the header's.  top < 0: the product's top digit
// is not reported (the last product, whose operand is the sum)
Fr30 mul(const Fr30& a, const Fr30& b, int top = kProdTop) {
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
// the kernel's sum: a + b digit-wise, carry-normalised; the raw digits reported in 64 bits, wrapped to 32 as the device would
Fr30 add(const Fr30& a, const Fr30& b) {
    Fr30 r;
    for (int i = 0; i < kR9; i++) {
        const int64_t s = (int64_t)a.d[i] + (int64_t)b.d[i];
        if (i < kR9 - 1) see(kRaw, s);
        r.d[i] = (int32_t)(uint32_t)(uint64_t)s;
    }
    r = fr30_norm(r);
    digits(r, kTop);
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
Fr30 read_image() {
    char h[80];
    uint32_t l[8] = {};
    ok = ok && scanf("%79s", h) == 1 && hex_limbs(h, l);
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
kzg_host::Fr pow2(int k) {
    kzg_host::Fr v = kzg_host::kFrOne;
    for (int i = 0; i < k; i++) v = kzg_host::fr_add(v, v);
    return v;
}

constexpr int kMaxT = 7, kMaxG = 8;

}  // namespace

int main() {
    int K = 0;
    if (scanf("%d", &K) != 1 || K < 1 || K > 4096) return 2;
    const Fr30 k14 = fr30_arg_from_mont256(pow2(14));  // as cg_enqueue (api.hip) prepares it
    std::vector<Fr30> out;
    for (int k = 0; k < K; k++) {
        int t = 0, g = 0, p[kMaxG][kMaxT];
        if (scanf("%d %d", &t, &g) != 2 || t < 1 || t > kMaxT || g < 1 || g > kMaxG) return 2;
        for (int s = 0; s < g; s++)
            for (int j = 0; j < t; j++)
                if (scanf("%d", &p[s][j]) != 1 || p[s][j] < 0 || p[s][j] > 7) return 2;
        Fr30 f[kMaxT], qx[kMaxG];
        for (int j = 0; j < t; j++) f[j] = read_image();
        for (int s = 0; s < g; s++) qx[s] = read_image();
        if (!ok) return 2;
        Fr30 sum = fr30_zero();
        for (int s = 0; s < g; s++) {
            Fr30 acc = qx[s];
            for (int j = 0; j < t; j++) {
                if (!p[s][j]) continue;
                const Fr30 W = mul(f[j], k14);
                for (int e = 0; e < p[s][j]; e++) acc = mul(acc, W);
            }
            sum = add(sum, acc);
        }
        out.push_back(mul(sum, fr30_const_one270()));
    }
    for (int i = 0; i < kReports; i++) printf("%llu%c", (unsigned long long)rep[i], i + 1 < kReports ? ' ' : '\n');
    for (const Fr30& v : out) print(v);
    return 0;
}
