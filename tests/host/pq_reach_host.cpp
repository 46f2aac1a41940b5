// Host replay of k_pq_constraints' arithmetic (csrc/quotient_kernels.hip) on the unchanged csrc/fr30.hip.h, for
// tests/test_perm_quotient.py: a stand-alone program (plain g++ -fwrapv; the header is __host__ __device__ code).  Test
// infrastructure only.
//
// It replays one coset point per input line in the kernel's order of products, sums and carry passes -- S = G + alpha^2 (z - 1) L0,
// the two running products over the t columns, S += alpha (A - B), the product with 1 / Z_H -- not the memory layout.  The twiddle
// w_N^i and 1 / Z_H are INPUTS, so the test can make them extremal.
//
// stdin:   t K has_gate
//          alpha beta gamma bkg_0 .. bkg_(t-1)        (blst_fr images, 64 hex digits each; alpha and beta are plain scalars' images,
//                                                      bkg_j = beta k_j g)
//          K lines:  w zinv z zrot l0 gate f_0 .. f_(t-1) s_0 .. s_(t-1)      (w, zinv: images of the plain multipliers; the rest
//                                                                              images; gate is read and ignored without has_gate)
// stdout:  thirteen numbers.  For each of the five sums of the kernel, in the order f + gamma, the factors a_j / b_j, D = A - B,
//          z - one, S: the largest |digit 0..7| entering its carry pass as a raw sum or difference (five numbers), then the
//          largest |digit 8| leaving it (five numbers).  Then the largest |digit 0..7| leaving any carry pass, load or product,
//          the largest |digit 8| of any product, the largest |column| of any product (exact, saturated at 2^64 - 1).
//          Then the K results.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../kzg_poly_commit_exploration_amd/csrc/fr30.hip.h"
#include "../../kzg_poly_commit_exploration_amd/csrc/host_fr.hpp"
#include "../../kzg_poly_commit_exploration_amd/csrc/fr30_host.hpp"

using namespace kzg;

namespace {

enum Sum { kFg = 0, kFactor, kD, kZ1, kS, kSums };
enum { kRaw = 0, kTop = kSums, kNorm = 2 * kSums, kProdTop, kColumn, kReports };
uint64_t rep[kReports];
void see(int which, int64_t v) {
    const uint64_t m = v < 0 ? (uint64_t)(-v) : (uint64_t)v;
    if (m > rep[which]) rep[which] = m;
}
// digits 0..7 of a normalised value, a load or a product; the top digit goes to `top` (-1: not reported, a canonical load)
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
    return p;
}
// sum `which` of the kernel: a + sign b digit-wise, carry-normalised; the raw digits reported in 64 bits, wrapped to 32 as the
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
Fr30 image_of(const kzg_host::Fr& w) {
    uint32_t l[8];
    memcpy(l, w.l, 32);
    const Fr30 v = fr30_from_limbs(l);
    digits(v, -1);
    return v;
}
Fr30 read_image() { return image_of(read_fr()); }
Fr30 read_multiplier() { return fr30_arg_from_mont256(read_fr()); }
// a stored multiplier: the canonical 8 x u32 of the x 2^270 form, loaded like a value
Fr30 read_stored_multiplier() {
    kzg_host::Fr k14 = kzg_host::kFrOne;
    for (int i = 0; i < 14; i++) k14 = kzg_host::fr_add(k14, k14);
    return image_of(kzg_host::fr_mul(read_fr(), k14));
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

constexpr int kMaxT = 7;

}  // namespace

int main() {
    int t = 0, K = 0, has_gate = 0;
    if (scanf("%d %d %d", &t, &K, &has_gate) != 3 || t < 1 || t > kMaxT || K < 1 || K > 4096) return 2;
    const kzg_host::Fr alpha = read_fr(), beta = read_fr();
    const Fr30 gamma = read_image();
    Fr30 bkg[kMaxT];
    for (int j = 0; j < t; j++) bkg[j] = read_image();
    if (!ok) return 2;
    // as PqKernelScalars (api.hip) prepares them
    const Fr30 f_beta = fr30_arg_from_mont256(beta);
    const Fr30 a1 = fr30_arg_from_mont256(kzg_host::fr_mul(alpha, pow2(14 * t)));
    const Fr30 a2 = fr30_arg_from_mont256(kzg_host::fr_mul(kzg_host::fr_mul(alpha, alpha), pow2(14)));
    const Fr30 one = image_of(kzg_host::kFrOne);
    std::vector<Fr30> out;
    for (int k = 0; k < K; k++) {
        const Fr30 w = read_multiplier(), zinv = read_stored_multiplier();
        const Fr30 zi = read_image(), zr = read_image(), l0 = read_image(), gate = read_image();
        Fr30 f[kMaxT], s[kMaxT];
        for (int j = 0; j < t; j++) f[j] = read_image();
        for (int j = 0; j < t; j++) s[j] = read_image();
        if (!ok) return 2;
        Fr30 sum = mul(mul(add(kZ1, zi, one, -1), l0), a2);
        if (has_gate) sum = add(kS, gate, sum);
        Fr30 a = zi, b = zr;
        for (int j = 0; j < t; j++) {
            const Fr30 fg = add(kFg, f[j], gamma);
            a = mul(a, add(kFactor, fg, mul(bkg[j], w)));
            b = mul(b, add(kFactor, fg, mul(s[j], f_beta)));
        }
        sum = add(kS, sum, mul(add(kD, a, b, -1), a1));
        out.push_back(mul(sum, zinv));
    }
    for (int i = 0; i < kReports; i++) printf("%llu%c", (unsigned long long)rep[i], i + 1 < kReports ? ' ' : '\n');
    for (const Fr30& v : out) print(v);
    return 0;
}
